"""The key-frame database on the device (vo_bow_vector, vo_kfdb_*) against tests/kfdb_ref.py: exact equality of the
candidate ids, their order, the counts and the score bits."""
import ctypes as C

import numpy as np
import pytest

import kfdb_inputs
import kfdb_ref

pytestmark = pytest.mark.gpu

NW = kfdb_inputs.N_WORDS
_scenes = {}


def scene_of(n):
    if n not in _scenes:
        _scenes[n] = kfdb_inputs.Scene(n)
    return _scenes[n]


def build_gpu(vo, scene, n=None, max_batch=1024, max_kf=None, max_wpk=256):
    n = scene.n_kf if n is None else n
    db = vo.KeyFrameDatabase(NW, max_kf or max(n, 1), max_wpk, max_batch)
    for i in range(n):
        assert db.insert(*scene.vectors[i]) == i
    for i in range(n):
        db.set_neighbors(i, [j for j in scene.neighbors[i] if j < n])
    return db


def ref_reloc(ref, queries, stale=None):
    out = [ref.query_reloc(*q, stale=stale) for q in queries]
    rows = np.array([r for _, r in out], np.float32).reshape(len(queries), len(ref.kfs))
    return [np.array(c, np.int32) for c, _ in out], rows


def ref_loop(ref, lqs, explicit=None):
    out = [ref.query_loop(*lq["vector"], lq["excluded"], min_score=None if explicit is None else explicit[i],
                          connected=lq["connected"]) for i, lq in enumerate(lqs)]
    rows = np.array([r for _, r in out], np.float32).reshape(len(lqs), len(ref.kfs))
    return [np.array(c, np.int32) for c, _ in out], rows


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), (g, w)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n", kfdb_inputs.SIZES)
@pytest.mark.parametrize("batch", (1, 7, 1024))
def test_queries_match_reference(vo, n, batch):
    scene = scene_of(n)
    ref = kfdb_inputs.build_ref(scene)
    db = build_gpu(vo, scene)
    assert len(db) == n
    # a scene to draw lost frames from even when the database is empty or tiny
    src = scene if n >= 37 else scene_of(37)
    queries = src.reloc_queries(batch, seed=n)
    stale = np.random.default_rng(n).random(n).astype(np.float32) * (np.random.default_rng(n + 1).random(n) < 0.5)
    for st in (None, stale):
        got, rows = db.query_reloc(queries, stale_score=st, max_out=64, scores=True)
        want, wrows = ref_reloc(ref, queries, st)
        same(got, want)
        assert np.array_equal(bits(rows), bits(wrows))
    lqs = scene.loop_queries(batch)
    if lqs:
        got, rows = db.query_loop([q["vector"] for q in lqs], [q["excluded"] for q in lqs], connected=[q["connected"] for q in lqs],
                                  scores=True)
        # (one set of reference answers serves the computed and the explicit min_score: the reference is given the value)
        ms = [ref.min_score(*q["vector"], q["connected"]) for q in lqs]
        want, wrows = ref_loop(ref, lqs, explicit=ms)
        same(got, want)
        assert np.array_equal(bits(rows), bits(wrows))
        # min_score == NULL equals the explicit value
        got2, rows2 = db.query_loop([q["vector"] for q in lqs], [q["excluded"] for q in lqs], min_score=ms, scores=True)
        same(got2, want)
        assert np.array_equal(bits(rows2), bits(wrows))
        # a demanding explicit min_score (the scored list can end up empty)
        hi = [np.float32(0.35)] * len(lqs)
        got3, rows3 = db.query_loop([q["vector"] for q in lqs], [q["excluded"] for q in lqs], min_score=hi, scores=True)
        want3, wrows3 = ref_loop(ref, lqs, explicit=hi)
        same(got3, want3)
        assert np.array_equal(bits(rows3), bits(wrows3))
    db.close()


def test_bow_vector_matches_reference(vo):
    rng = np.random.default_rng(11)
    scene = scene_of(37)
    frames = [scene.frame_features(p % scene.n_places) for p in range(20)]
    frames.append((np.zeros(0, np.int32), np.zeros(0)))
    w = rng.integers(0, 900, 3000).astype(np.int32)               # beyond the kernel's LDS form
    frames.append((w, np.where(rng.random(3000) < 0.1, 0.0, rng.uniform(0.1, 5.0, 3000))))
    frames.append((np.array([5, 5, 9], np.int32), np.array([0.0, -1.0, 0.0])))   # only skipped features
    for batch in (frames[:1], frames[:7], frames):
        got = vo.bow_vector([f[0] for f in batch], [f[1] for f in batch])
        for (gw, gv), f in zip(got, batch):
            ww, wv = kfdb_ref.bow_vector(*f)
            assert np.array_equal(gw, ww) and np.array_equal(gv.view(np.uint64), wv.view(np.uint64))


def test_dev_forms_equal_host_forms(vo):
    import torch
    scene = scene_of(500)
    dev = torch.device("cuda:0")
    db = build_gpu(vo, scene)
    queries = scene.reloc_queries(33)
    host_c, host_rows = db.query_reloc(queries, max_out=64, scores=True)
    qs, qw = vo._csr([q[0] for q in queries], np.int32)
    _, qv = vo._csr([q[1] for q in queries], np.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n_cand = torch.zeros(33, dtype=torch.int32, device=dev)
    cand = torch.zeros((33, 64), dtype=torch.int32, device=dev)
    rows = torch.zeros((33, 500), dtype=torch.float32, device=dev)
    tq = (t(qs), t(qw), t(qv))
    db.query_reloc_dev(33, *tq, None, 64, n_cand, cand, rows)
    torch.cuda.synchronize()
    nc, cd = n_cand.cpu().numpy(), cand.cpu().numpy()
    same([cd[i, :nc[i]] for i in range(33)], host_c)
    assert np.array_equal(bits(rows.cpu().numpy()), bits(host_rows))
    # loop
    lqs = scene.loop_queries(21)
    host_c, host_rows = db.query_loop([q["vector"] for q in lqs], [q["excluded"] for q in lqs], connected=[q["connected"] for q in lqs],
                                      scores=True)
    qs, qw = vo._csr([q["vector"][0] for q in lqs], np.int32)
    _, qv = vo._csr([q["vector"][1] for q in lqs], np.float64)
    es, ex = vo._csr([q["excluded"] for q in lqs], np.int32)
    cs, cn = vo._csr([q["connected"] for q in lqs], np.int32)
    n_cand = torch.zeros(21, dtype=torch.int32, device=dev)
    rows = torch.zeros((21, 500), dtype=torch.float32, device=dev)
    db.query_loop_dev(21, t(qs), t(qw), t(qv), t(es), t(ex), None, t(cs), t(cn), 64, n_cand, cand, rows)
    torch.cuda.synchronize()
    nc, cd = n_cand.cpu().numpy(), cand.cpu().numpy()
    same([cd[i, :nc[i]] for i in range(21)], host_c)
    assert np.array_equal(bits(rows.cpu().numpy()), bits(host_rows))
    # vo_bow_vector_dev and vo_kfdb_insert_dev: a second database filled from device vectors answers alike
    feats = scene.features[:40]
    fs, fw = vo._csr([f[0] for f in feats], np.int32)
    _, fx = vo._csr([f[1] for f in feats], np.float64)
    o_s = torch.zeros(41, dtype=torch.int32, device=dev)
    o_w = torch.zeros(len(fw), dtype=torch.int32, device=dev)
    o_v = torch.zeros(len(fw), dtype=torch.float64, device=dev)
    vo.bow_vector_dev(40, len(fw), t(fs), t(fw), t(fx), o_s, o_w, o_v)
    torch.cuda.synchronize()
    s = o_s.cpu().numpy()
    host = vo.bow_vector([f[0] for f in feats], [f[1] for f in feats])
    db2, db3 = vo.KeyFrameDatabase(NW, 64, 256, 64), vo.KeyFrameDatabase(NW, 64, 256, 64)
    for k in range(40):
        assert np.array_equal(o_w[s[k]:s[k + 1]].cpu().numpy(), host[k][0])
        assert np.array_equal(o_v[s[k]:s[k + 1]].cpu().numpy().view(np.uint64), host[k][1].view(np.uint64))
        assert db2.insert(o_w[s[k]:s[k + 1]], o_v[s[k]:s[k + 1]]) == k
        assert db3.insert(*host[k]) == k
    a, ra = db2.query_reloc(queries, scores=True)
    b, rb = db3.query_reloc(queries, scores=True)
    same(a, b)
    assert np.array_equal(bits(ra), bits(rb))
    for d in (db, db2, db3):
        d.close()


def test_batch_invariance(vo):
    scene = scene_of(500)
    db = build_gpu(vo, scene)
    queries = scene.reloc_queries(64, seed=3)
    stale = np.random.default_rng(8).random(500).astype(np.float32)
    base, rows = db.query_reloc(queries, stale_score=stale, scores=True)
    perm = np.random.default_rng(9).permutation(64)
    got, prow = db.query_reloc([queries[i] for i in perm], stale_score=stale, scores=True)
    same(got, [base[i] for i in perm])
    assert np.array_equal(bits(prow), bits(rows[perm]))
    for i in range(64):
        one, r1 = db.query_reloc([queries[i]], stale_score=stale, scores=True)
        assert np.array_equal(one[0], base[i]) and np.array_equal(bits(r1[0]), bits(rows[i]))
    lqs = scene.loop_queries(32)
    args = lambda qs: ([q["vector"] for q in qs], [q["excluded"] for q in qs])
    base = db.query_loop(*args(lqs), connected=[q["connected"] for q in lqs])
    perm = np.random.default_rng(10).permutation(32)
    pl = [lqs[i] for i in perm]
    same(db.query_loop(*args(pl), connected=[q["connected"] for q in pl]), [base[i] for i in perm])
    for i in range(32):
        assert np.array_equal(db.query_loop(*args([lqs[i]]), connected=[lqs[i]["connected"]])[0], base[i])
    db.close()


def test_inserts_interleaved_with_queries_and_changed_neighbors(vo):
    scene = scene_of(500)
    db = vo.KeyFrameDatabase(NW, 500, 256, 16)
    ref = kfdb_ref.Database()
    queries = scene.reloc_queries(16, seed=5)
    assert all(len(c) == 0 for c in db.query_reloc(queries))           # nothing inserted yet
    k = 0
    for upto in (1, 2, 40, 41, 200, 500):
        while k < upto:
            assert db.insert(*scene.vectors[k]) == ref.insert(*scene.vectors[k]) == k
            nb = [j for j in scene.neighbors[k] if j <= k and j != k]
            db.set_neighbors(k, nb), ref.set_neighbors(k, nb)
            k += 1
        got, rows = db.query_reloc(queries, scores=True)
        want, wrows = ref_reloc(ref, queries)
        same(got, want)
        assert np.array_equal(bits(rows), bits(wrows))
    # neighbours changed between two queries
    for i in range(0, 500, 3):
        nb = [j for j in scene.neighbors[(i * 7) % 500]][:6]
        db.set_neighbors(i, nb), ref.set_neighbors(i, nb)
    same(db.query_reloc(queries), ref_reloc(ref, queries)[0])
    lqs = scene.loop_queries(16)
    same(db.query_loop([q["vector"] for q in lqs], [q["excluded"] for q in lqs], connected=[q["connected"] for q in lqs]),
         ref_loop(ref, lqs)[0])
    db.close()


def test_sequential_use_with_carried_scores(vo):
    """the shim's use: one frame per call, stale_score = what the previous calls left (score_out), against the reference
    with its members carried from query to query"""
    scene = scene_of(500)
    db, ref = build_gpu(vo, scene, max_batch=1), kfdb_inputs.build_ref(scene)
    stale = np.zeros(500, np.float32)
    n_stale = 0
    for fid, q in enumerate(scene.reloc_queries(120), start=1):
        want = ref.detect_reloc(fid, *q)
        n_stale += ref.trace.get("stale_nonzero", 0)
        got, rows = db.query_reloc([q], stale_score=stale, scores=True)
        assert np.array_equal(got[0], np.array(want, np.int32))
        stale = rows[0]
        assert np.array_equal(bits(stale), bits(ref.reloc_scores()))
    assert n_stale > 0
    db.close()


def test_capacity_paths(vo):
    scene = scene_of(37)
    db = build_gpu(vo, scene, max_batch=4, max_kf=37, max_wpk=256)
    ref = kfdb_inputs.build_ref(scene)
    L = vo.lib()
    with pytest.raises(vo.VoError, match="status -4"):                 # max_keyframes
        db.insert(*scene.vectors[0])
    assert len(db) == 37
    queries = scene.reloc_queries(8)
    with pytest.raises(vo.VoError, match="status -4"):                 # max_batch
        db.query_reloc(queries)
    big = (np.arange(300, dtype=np.int32), np.full(300, 1 / 300))
    with pytest.raises(vo.VoError, match="status -4"):                 # max_words_per_keyframe (query side)
        db.query_reloc([big])
    small = vo.KeyFrameDatabase(NW, 4, 16, 4)
    with pytest.raises(vo.VoError, match="status -4"):                 # max_words_per_keyframe (insert side)
        small.insert(*scene.vectors[0])
    assert len(small) == 0
    small.close()
    # max_out: the status says so, n_cand still holds the true counts, the first max_out candidates are in place
    qs = [q for q in queries if len(ref.query_reloc(*q)[0]) >= 2][:4]
    assert qs
    want = [ref.query_reloc(*q)[0] for q in qs]
    with pytest.raises(vo.VoError, match="status -4") as e:
        db.query_reloc(qs, max_out=1)
    assert list(e.value.args[1]) == [len(w) for w in want]
    s, w = vo._csr([q[0] for q in qs], np.int32)
    _, v = vo._csr([q[1] for q in qs], np.float64)
    nc, cd = np.zeros(len(qs), np.int32), np.full((len(qs), 1), -7, np.int32)
    assert L.vo_kfdb_query_reloc(db._h, len(qs), vo._p(s), vo._p(w), vo._p(v), None, 1, vo._p(nc), vo._p(cd), None) == -4
    assert list(nc) == [len(x) for x in want] and [int(c) for c in cd[:, 0]] == [x[0] for x in want]
    db.close()
    assert L.vo_kfdb_create(C.byref(C.c_void_p()), NW, 1 << 20, 1 << 12, 4) == -4      # beyond the 32-bit index range


def test_invalid_arguments_are_refused(vo):
    L = vo.lib()
    h = C.c_void_p()
    for args in ((0, 4, 4, 4), (10, 0, 4, 4), (10, 4, 0, 4), (10, 4, 4, 0)):
        assert L.vo_kfdb_create(C.byref(h), *args) == -1
    assert L.vo_kfdb_create(None, 10, 4, 4, 4) == -1
    db = vo.KeyFrameDatabase(100, 8, 8, 4)
    i32, f64 = lambda *a: np.array(a, np.int32), lambda *a: np.array(a, np.float64)
    for w in (i32(3, 3), i32(5, 2), i32(-1, 2), i32(1, 100)):             # not strictly ascending / out of range
        with pytest.raises(vo.VoError, match="status -1"):
            db.insert(w, f64(0.5, 0.5))
    assert len(db) == 0
    assert db.insert(i32(1, 2), f64(0.5, 0.5)) == 0 and db.insert(i32(2, 9), f64(0.5, 0.5)) == 1
    for kf, ids in ((2, [0]), (-1, [0]), (0, [2]), (0, [-1]), (0, list(range(11)))):
        with pytest.raises(vo.VoError, match="status -1"):
            db.set_neighbors(kf, ids)
    nc, cd = np.zeros(1, np.int32), np.zeros(4, np.int32)
    s, w, v = i32(0, 2), i32(1, 2), f64(0.5, 0.5)      # (named: the arrays must outlive the raw pointers)
    q = (vo._p(s), vo._p(w), vo._p(v))
    assert L.vo_kfdb_query_reloc(None, 1, *q, None, 4, vo._p(nc), vo._p(cd), None) == -1
    assert L.vo_kfdb_query_reloc(db._h, -1, *q, None, 4, vo._p(nc), vo._p(cd), None) == -1
    assert L.vo_kfdb_query_reloc(db._h, 1, *q, None, -1, vo._p(nc), vo._p(cd), None) == -1
    assert L.vo_kfdb_query_reloc(db._h, 1, *q, None, 4, None, vo._p(cd), None) == -1
    assert L.vo_kfdb_query_reloc(db._h, 1, *q, None, 4, vo._p(nc), None, None) == -1
    bad, s1 = i32(1, 100), i32(1, 2)
    assert L.vo_kfdb_query_reloc(db._h, 1, vo._p(s), vo._p(bad), q[2], None, 4, vo._p(nc), vo._p(cd), None) == -1   # word out of range
    assert L.vo_kfdb_query_reloc(db._h, 1, vo._p(s1), q[1], q[2], None, 4, vo._p(nc), vo._p(cd), None) == -1         # CSR not from 0
    es, e0, e5, ms = i32(0, 1), i32(0), i32(5), np.zeros(1, np.float32)
    assert L.vo_kfdb_query_loop(db._h, 1, *q, None, None, None, None, None, 4, vo._p(nc), vo._p(cd), None) == -1     # no exclusion list
    assert L.vo_kfdb_query_loop(db._h, 1, *q, vo._p(es), vo._p(e0), None, None, None, 4, vo._p(nc), vo._p(cd), None) == -1  # no min_score, no conn
    assert L.vo_kfdb_query_loop(db._h, 1, *q, vo._p(es), vo._p(e5), vo._p(ms), None, None, 4, vo._p(nc), vo._p(cd), None) == -1  # excluded id out of range
    assert L.vo_kfdb_set_option(db._h, 99, 1) == -1 and L.vo_kfdb_size(None) == -1
    assert L.vo_bow_vector(1, None, None, None, None, None, None) == -1 and L.vo_bow_vector(-1, None, None, None, None, None, None) == -1
    assert db.query_reloc([(i32(1, 2), f64(0.5, 0.5))])[0].tolist() == [0]    # the handle still works
    db.close()


def test_global_slab_fallback_gives_the_same_results(vo):
    scene = scene_of(500)
    db = build_gpu(vo, scene)
    queries, lqs = scene.reloc_queries(40, seed=7), scene.loop_queries(24)
    stale = np.random.default_rng(3).random(500).astype(np.float32)
    largs = ([q["vector"] for q in lqs], [q["excluded"] for q in lqs])
    a = db.query_reloc(queries, stale_score=stale, scores=True)
    la = db.query_loop(*largs, connected=[q["connected"] for q in lqs], scores=True)
    db.set_option(db.OPT_LDS_KEYFRAMES, 64)            # 500 key-frames no longer fit: counters in the device-memory slab
    b = db.query_reloc(queries, stale_score=stale, scores=True)
    lb = db.query_loop(*largs, connected=[q["connected"] for q in lqs], scores=True)
    same(a[0], b[0]), same(la[0], lb[0])
    assert np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(la[1]), bits(lb[1]))
    same(b[0], ref_reloc(kfdb_inputs.build_ref(scene), queries, stale)[0])
    db.close()


def test_more_keyframes_than_the_default_lds_allowance(vo):
    """7000 small key-frames: the counters need more LDS than a launch gets by default (the kernel asks for it, or falls
    back to the device-memory slab); same answers as the reference"""
    rng = np.random.default_rng(21)
    n = 7000
    db, ref = vo.KeyFrameDatabase(500, n, 8, 8), kfdb_ref.Database()
    for k in range(n):
        w = np.sort(rng.choice(500, 4, replace=False)).astype(np.int32)
        v = rng.random(4)
        v /= v.sum()
        assert db.insert(w, v) == ref.insert(w, v) == k
    for k in range(0, n, 50):
        nb = [int(j) for j in rng.choice(n, 6, replace=False) if j != k]
        db.set_neighbors(k, nb), ref.set_neighbors(k, nb)
    queries = []
    for _ in range(8):
        w = np.sort(rng.choice(500, 6, replace=False)).astype(np.int32)
        queries.append((w, np.full(6, 1 / 6)))
    got, rows = db.query_reloc(queries, max_out=4096, scores=True)
    want, wrows = ref_reloc(ref, queries)
    same(got, want)
    assert np.array_equal(bits(rows), bits(wrows))
    db.close()


def test_batched_set_neighbors_equals_one_by_one(vo):
    scene = scene_of(500)
    a = build_gpu(vo, scene)                               # vo_kfdb_set_neighbors per key-frame
    b = vo.KeyFrameDatabase(NW, 500, 256, 64)
    for i in range(500):
        b.insert(*scene.vectors[i])
    b.set_neighbors_batch(0, scene.neighbors[:200])
    b.set_neighbors_batch(200, scene.neighbors[200:])
    b.set_neighbors_batch(7, [scene.neighbors[7]])         # a span of one, again
    queries = scene.reloc_queries(64, seed=12)
    ga, ra = a.query_reloc(queries, scores=True)
    gb, rb = b.query_reloc(queries, scores=True)
    same(ga, gb)
    assert np.array_equal(bits(ra), bits(rb))
    same(gb, ref_reloc(kfdb_inputs.build_ref(scene), queries)[0])
    n, ids = np.array([11], np.int32), np.zeros((1, 10), np.int32)
    L = vo.lib()
    assert L.vo_kfdb_set_neighbors_batch(b._h, 0, 1, vo._p(n), vo._p(ids)) == -1          # more than 10
    n[0], ids[0, 0] = 1, 500
    assert L.vo_kfdb_set_neighbors_batch(b._h, 0, 1, vo._p(n), vo._p(ids)) == -1          # id out of range
    assert L.vo_kfdb_set_neighbors_batch(b._h, 499, 2, vo._p(n), vo._p(ids)) == -1        # span beyond the database
    same(b.query_reloc(queries), gb)                                                       # refused calls changed nothing
    a.close(), b.close()
