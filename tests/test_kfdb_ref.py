"""CPU checks of the key-frame database's reference (tests/kfdb_ref.py) and of the fixture (tests/kfdb_inputs.py): the
restatement against an independent dense formulation, and the branches the fixture has to reach -- asserted with the
reference alone, so that the GPU comparison of tests/test_gpu_kfdb.py means something."""
import numpy as np
import pytest

import kfdb_inputs
import kfdb_ref

F32 = np.float32


@pytest.fixture(scope="module")
def scene():
    return kfdb_inputs.Scene(500)


def _dense(scene, n):
    """entries of all key-frame vectors as flat arrays (key-frame id, word)"""
    kid = np.concatenate([np.full(len(scene.vectors[k][0]), k) for k in range(n)])
    wrd = np.concatenate([scene.vectors[k][0] for k in range(n)])
    return kid, wrd


def _orc_score(orc, q, c):
    return orc.lib().orc_bow_score(len(q[0]), np.ascontiguousarray(q[0], np.int32), np.ascontiguousarray(q[1]), len(c[0]),
                                   np.ascontiguousarray(c[0], np.int32), np.ascontiguousarray(c[1]))


def test_reference_against_dense_formulation(scene, orc):
    n = scene.n_kf
    db = kfdb_inputs.build_ref(scene)
    kid, wrd = _dense(scene, n)
    for q in scene.reloc_queries(60):
        cands, row = db.query_reloc(*q)
        tr = db.trace
        # counts: one row of the (queries x words) . (words x key-frames) product
        hit = np.isin(wrd, q[0])
        counts = np.bincount(kid[hit], minlength=n)
        firstw = np.full(n, np.iinfo(np.int64).max)
        np.minimum.at(firstw, kid[hit], wrd[hit])
        sharing = [int(k) for k in sorted(np.nonzero(counts)[0], key=lambda k: (firstw[k], k))]
        assert sharing == tr["sharing"]
        if not sharing:
            assert cands == []
            continue
        mx = counts.max()
        assert mx == tr["max_common"]
        scored = [k for k in sharing if counts[k] > int(0.8 * mx)]
        assert scored == tr["scored"]
        for k in scored:
            assert row[k] == F32(_orc_score(orc, q, scene.vectors[k]))
        # groups from the dense rows
        s = np.zeros(n, np.float32)
        s[scored] = row[scored]
        groups = []
        for k in scored:
            g, best, rep = s[k], s[k], k
            for m in scene.neighbors[k]:
                if counts[m] > 0:
                    g = F32(g + s[m])
                    if s[m] > best:
                        best, rep = s[m], m
            groups.append((g, rep))
        top = max([g for g, _ in groups] + [F32(0)])
        want = []
        for g, rep in groups:
            if g > F32(0.75) * top and rep not in want:
                want.append(rep)
        assert want == cands


def test_loop_reference_against_dense_formulation(scene, orc):
    n = scene.n_kf
    db = kfdb_inputs.build_ref(scene)
    kid, wrd = _dense(scene, n)
    for lq in scene.loop_queries(40):
        q = lq["vector"]
        ms = db.min_score(*q, lq["connected"])
        assert ms == min([F32(1.0)] + [F32(_orc_score(orc, q, scene.vectors[c])) for c in lq["connected"]])
        cands, row = db.query_loop(*q, lq["excluded"], connected=lq["connected"])
        hit = np.isin(wrd, q[0]) & ~np.isin(kid, lq["excluded"])
        counts = np.bincount(kid[hit], minlength=n)
        if counts.max() == 0:
            assert cands == []
            continue
        mn = int(F32(0.8) * F32(counts.max()))
        scored = np.nonzero(counts > mn)[0]
        assert sorted(db.trace["scored_all"]) == list(scored)
        for k in scored:
            assert row[k] == F32(_orc_score(orc, q, scene.vectors[k]))
        assert np.all(row[np.setdiff1d(np.arange(n), scored)] == -1.0)
        assert all(row[k] >= ms for k in db.trace["scored"])
        # the group stage, the 0.75 gate and the de-duplication from the dense rows
        firstw = np.full(n, np.iinfo(np.int64).max)
        np.minimum.at(firstw, kid[hit], wrd[hit])
        entered = [int(k) for k in sorted(scored, key=lambda k: (firstw[k], k)) if row[k] >= ms]
        assert entered == db.trace["scored"]
        groups, top = [], ms
        for k in entered:
            g, best, rep = row[k], row[k], k
            for m in scene.neighbors[k]:
                if counts[m] > mn:
                    g = F32(g + row[m])
                    if row[m] > best:
                        best, rep = row[m], m
            groups.append((g, rep))
            if g > top:
                top = g
        want = []
        for g, rep in groups:
            if g > F32(0.75) * top and rep not in want:
                want.append(rep)
        assert want == cands


def test_fixture_reaches_every_branch(scene):
    """a condition on the inputs, found with the reference alone"""
    db = kfdb_inputs.build_ref(scene)
    seen = dict(gate08=0, stale_nonzero=0, stale_zero=0, rep_other=0, duplicate=0, gate075=0, early_sharing=0)
    reloc_max = set()
    fid = 0
    for q in scene.reloc_queries(120):          # sequential use: members carried from query to query
        fid += 1
        cands = db.detect_reloc(fid, *q)
        tr = db.trace
        if tr["early"] == "sharing":
            seen["early_sharing"] += 1
            assert cands == []
            continue
        assert tr["early"] is None                # the key-frame with the most shared words always passes the 0.8 gate
        reloc_max.add(tr["max_common"])
        seen["gate08"] += len(tr["sharing"]) > len(tr["scored"])
        seen["stale_nonzero"] += tr["stale_nonzero"]
        seen["stale_zero"] += tr["stale_zero"]
        seen["rep_other"] += any(rep != k for (_, rep), k in zip(tr["groups"], tr["scored"]))
        seen["duplicate"] += tr["duplicates"]
        seen["gate075"] += any(g <= tr["keep"] for g, _ in tr["groups"])
    assert all(v > 0 for v in seen.values()), seen

    lseen = dict(min_score_gate=0, excluded_most=0, early_sharing=0, early_scored=0, gate075=0, duplicate=0)
    loop_max = set()
    kid = 0
    for lq in scene.loop_queries(80):
        kid += 1
        ms = db.min_score(*lq["vector"], lq["connected"])
        cands = db.detect_loop(kid, *lq["vector"], lq["excluded"], ms)
        tr = db.trace
        if tr["early"] == "sharing":
            lseen["early_sharing"] += 1
            continue
        loop_max.add(tr["max_common"])
        lseen["excluded_most"] += max(tr["excluded_shared"].values(), default=0) > 0 and \
            len(lq["vector"][0]) > tr["max_common"] and lq["kf"] in tr["excluded_shared"]
        lseen["min_score_gate"] += len(tr["scored_all"]) > len(tr["scored"])
        if tr["early"] == "scored":
            lseen["early_scored"] += 1
            assert cands == []
            continue
        lseen["gate075"] += any(g <= tr["keep"] for g, _ in tr["groups"])
        lseen["duplicate"] += tr["duplicates"]
    # an isolated key-frame (nothing else shares a word once its neighbourhood is excluded)
    one = kfdb_inputs.Scene(1)
    d1 = kfdb_inputs.build_ref(one)
    assert d1.detect_loop(1, *one.vectors[0], [0], F32(0.0)) == [] and d1.trace["early"] == "sharing"
    lseen["early_sharing"] += 1
    # every score below an explicit min_score
    lq = scene.loop_queries(1)[0]
    assert db.detect_loop(10_000, *lq["vector"], lq["excluded"], F32(0.999)) == [] and db.trace["early"] == "scored"
    lseen["early_scored"] += 1
    assert all(v > 0 for v in lseen.values()), lseen
    # the float and the double product 0.8 * max at the same max
    assert reloc_max & loop_max, (sorted(reloc_max), sorted(loop_max))


def test_empty_database_and_sizes():
    db = kfdb_ref.Database()
    assert db.detect_reloc(1, [1, 2], [0.5, 0.5]) == [] and db.trace["early"] == "sharing"
    assert db.detect_loop(1, [1, 2], [0.5, 0.5], [], F32(0.1)) == []
    assert kfdb_inputs.SIZES == (0, 1, 37, 500, 4096) and kfdb_inputs.N_WORDS == 10 ** 5


def test_bow_vector_against_dict_formulation():
    rng = np.random.default_rng(5)
    for n in (0, 1, 5, 300, 1500):
        words = rng.integers(0, max(n // 3, 2), n).astype(np.int32) * 7
        weights = np.where(rng.random(n) < 0.1, 0.0, rng.uniform(0.1, 9.0, n))
        if n >= 5:
            weights[3] = -1.0
        w, v = kfdb_ref.bow_vector(words, weights)
        acc = {}
        for a, b in zip(words.tolist(), weights.tolist()):
            if b > 0:
                acc[a] = acc.get(a, 0.0) + b
        keys = sorted(acc)
        norm = 0.0
        for k in keys:
            norm += abs(acc[k])
        want = [acc[k] / norm if norm > 0 else acc[k] for k in keys]
        assert w.tolist() == keys and v.tolist() == want
        assert np.all(np.diff(w) > 0) and (n == 0 or len(w) == 0 or abs(v.sum() - 1.0) < 1e-12)
