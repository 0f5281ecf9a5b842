"""vo_vocab_train / vo_vocab_train_dev / vo_vocab_tree / vo_vocab_save on the device against the numpy restatement of the
contract (tests/vocab_ref.py).  Everything but the idf's log is integer arithmetic, so the tree (child_start,
children, node_desc, word_id) and the info block are compared for EXACT equality; the weights are the same libm's log of
the same ratio on the same machine and are compared for equality too.  Batch invariance needs no device hook: the subtree
property is established on the CPU (tests/test_vocab_ref.py) and exact equality on every input here carries it over."""
import ctypes as C

import numpy as np
import pytest

import vocab_inputs as I
import vocab_ref as R

pytestmark = pytest.mark.gpu


def _same(tree, info, ref):
    for key in ("child_start", "children", "node_desc", "word_id"):
        a, b = np.asarray(tree[key]), np.asarray(ref[key])
        assert a.shape == b.shape, (key, a.shape, b.shape, info, ref["info"])
        if not np.array_equal(a, b):
            bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
            raise AssertionError((key, "first differing rows", bad[:5], len(bad), info, ref["info"]))
    assert info == ref["info"]
    assert tree["L"] == ref["L"]
    assert np.array_equal(tree["node_weight"], ref["node_weight"])  # math.log and the library's log: the same libm here


def info_words(tree):
    return int((tree["word_id"] >= 0).sum())


def _train_and_check(vo, desc, off, k, L, seed=0):
    ref = R.train(desc, off, k, L, seed)
    V, info = vo.train_vocabulary(desc, off, k, L, seed)
    print(f"n = {len(desc)}, k = {k}, L = {L}: {info}")
    tree = V.tree()
    _same(tree, info, ref)
    assert ref["info"]["n_capped"] == 0  # the cap is a condition: it must not bite on the fixtures
    return V, tree, ref


@pytest.mark.parametrize("k,L", I.KL)
@pytest.mark.parametrize("size", ["0", "1", "k", "k+1", "63", "64", "65", "1000", "20000"])
def test_uniform_sizes(vo, size, k, L):
    n = {"k": k, "k+1": k + 1}.get(size) if size in ("k", "k+1") else int(size)
    desc = I.uniform(n, seed=n + k)
    V, tree, ref = _train_and_check(vo, desc, I.offsets(n, 7), k, L, seed=3)
    if n == 0:
        assert len(tree["word_id"]) == 1 and len(tree["children"]) == 0
    V.close()


@pytest.mark.timeout(900)
def test_uniform_200000(vo):
    n = 200_000
    V, tree, ref = _train_and_check(vo, I.uniform(n, seed=11), I.offsets(n, 200), 10, 5, seed=1)
    V.close()


@pytest.mark.parametrize("k,L", I.KL)
@pytest.mark.parametrize("kind", ["clustered", "duplicates", "all_equal"])
def test_structured_inputs(vo, kind, k, L):
    n = 6000
    desc = getattr(I, kind)(n, seed=k)
    V, tree, ref = _train_and_check(vo, desc, I.offsets(n, 40), k, L, seed=9)
    if kind == "all_equal":
        assert len(tree["word_id"]) == L + 1 and info_words(tree) == 1  # sum == 0 at the first draw: a chain of single centres
    V.close()


@pytest.mark.parametrize("k,L", I.KL)
def test_extracted_descriptors(vo, k, L):
    ext = vo.OrbExtractor(1000, 1.2, 8, 20, 7)
    desc, off = I.extracted(ext, 6)
    ext.close()
    assert len(off) == 7 and len(desc) > 3000
    V, tree, ref = _train_and_check(vo, desc, off, k, L, seed=5)
    V.close()


def test_host_and_device_forms_agree_and_seeds_matter(vo):
    import torch
    n, k, L = 5000, 10, 4
    desc, off = I.clustered(n, seed=2), I.offsets(n, 25)
    Vh, ih = vo.train_vocabulary(desc, off, k, L, seed=17)
    st = torch.cuda.Stream()
    td, to = torch.from_numpy(desc).cuda(), torch.from_numpy(off).cuda()
    torch.cuda.synchronize()
    Vd, idv = vo.train_vocabulary(td, to, k, L, seed=17, stream=st.cuda_stream)
    Vd0, id0 = vo.train_vocabulary(td, to, k, L, seed=17, stream=None)
    th, tdv, td0 = Vh.tree(), Vd.tree(), Vd0.tree()
    assert ih == idv == id0
    for key in th:
        assert np.array_equal(th[key], tdv[key]) and np.array_equal(th[key], td0[key]), key
    V2, i2 = vo.train_vocabulary(desc, off, k, L, seed=18)
    t2 = V2.tree()
    assert t2["node_desc"].shape != th["node_desc"].shape or not np.array_equal(t2["node_desc"], th["node_desc"])
    V3, i3 = vo.train_vocabulary(desc, off, k, L, seed=17)
    t3 = V3.tree()
    assert i3 == ih and all(np.array_equal(t3[key], th[key]) for key in th)
    for v in (Vh, Vd, Vd0, V2, V3):
        v.close()


def test_save_load_round_trip_and_transform(vo, tmp_path):
    n, k, L = 8000, 10, 5
    desc = I.clustered(n, seed=4)
    V, tree, ref = _train_and_check(vo, desc, I.offsets(n, 30), k, L, seed=2)
    V.save(tmp_path / "trained.dbow3", k)
    V2, info2 = vo.load_vocabulary(tmp_path / "trained.dbow3")
    assert info2 == dict(n_nodes=len(tree["word_id"]), n_words=int((tree["word_id"] >= 0).sum()), k=k, L=L)
    t2 = V2.tree()
    for key in tree:
        assert np.array_equal(tree[key], t2[key]), key
    # the existing transform on a trained tree (leaves above level L, nodes with fewer than k children)
    assert (ref["level"][ref["word_id"] >= 0] < L).any() and (np.diff(ref["child_start"]) % k != 0).any()
    fresh = np.concatenate([I.uniform(2500, seed=77), I.clustered(2500, seed=4)])
    leaf = R.transform(ref, fresh)
    for handle in (V, V2):
        word, weight, _ = handle.transform(fresh, 3)
        assert np.array_equal(word, ref["word_id"][leaf]) and np.array_equal(weight, ref["node_weight"][leaf])
    V.close(), V2.close()


def test_trained_tree_is_a_drop_in_for_search_by_bow(vo, orc):
    """vo_match_bow between two shifted synth frames, their FeatureVectors taken through a trained tree: the oracle's matches"""
    from test_gpu_match import _frame_pair, _uright
    k0, d0, k1, d1, dx, dy = _frame_pair(orc, 1)
    train = np.ascontiguousarray(np.concatenate([d0, d1]))
    V, info = vo.train_vocabulary(train, np.array([0, len(d0), len(train)], np.int32), 6, 3, seed=0)
    _, _, na = V.transform(d0, 2)
    _, _, nb = V.transform(d1, 2)
    V.close()
    ur0, _ = _uright(k0, 1)
    ur1, _ = _uright(k1, 2)
    A = vo.FrameArrays(k0["x"], k0["y"], k0["octave"], k0["angle"], ur0, d0)
    B = vo.FrameArrays(k1["x"], k1["y"], k1["octave"], k1["angle"], ur1, d1)
    ones0, ones1 = np.ones(len(k0), np.uint8), np.ones(len(k1), np.uint8)
    n, match = vo.Matcher(0.75).searchByBoW(A, ones0, vo.BowNodes(na), B, ones1, vo.BowNodes(nb), True, True)
    oA = orc.FrameData(k0["x"], k0["y"], k0["octave"], k0["angle"], ur0, d0)
    oB = orc.FrameData(k1["x"], k1["y"], k1["octave"], k1["angle"], ur1, d1)
    ba, bb = orc.BowData(na), orc.BowData(nb)
    om = np.full(len(k0), -1, np.int32)
    on = orc.lib().orc_match_bow(C.byref(oA.c), ones0, C.byref(ba.c), C.byref(oB.c), ones1, C.byref(bb.c), 1, 0.75, 1, om)
    assert n == on and np.array_equal(match, om) and n > 50


def test_argument_errors_and_capacity(vo):
    lib = vo.lib()
    desc, off = I.uniform(100), I.offsets(100, 4)
    sentinel = 0x5EED
    info = vo.VocabTrainInfo()

    def call(n, d, ni, o, k, L):
        h = C.c_void_p(sentinel)
        rc = lib.vo_vocab_train(n, vo._p(d), ni, vo._p(o), k, L, C.c_uint64(0), C.byref(h), C.byref(info))
        assert h.value == sentinel  # *out untouched
        return rc

    assert call(100, desc, 4, off, 1, 5) == -1
    assert call(100, desc, 4, off, 10, 0) == -1
    assert call(-1, desc, 4, off, 10, 5) == -1
    assert call(100, desc, 4, off[::-1].copy(), 10, 5) == -1
    assert call(100, desc, 4, np.array([0, 30, 20, 60, 100], np.int32), 10, 5) == -1
    assert call(100, desc, 4, np.array([0, 20, 30, 60, 99], np.int32), 10, 5) == -1
    assert b"image_offsets" in lib.vo_last_error()
    assert call(100, desc, 4, off, 33, 5) == -4
    assert call(100, desc, 4, off, 10, 17) == -4
    assert call((1 << 23) + 1, desc, 4, off, 10, 5) == -4
    assert b"exceed" in lib.vo_last_error()
    assert lib.vo_vocab_tree(None, None, None, None, None, None, None, None) == -1
    assert lib.vo_vocab_save(None, 10, b"/nonexistent") == -1


@pytest.mark.timeout(600)
def test_vo_run_harness_saves_a_vocabulary(vo, tmp_path):
    """examples/vo_run_hip.cpp --vocabulary-out: the run ends the way vo_run.cpp:234 does, and the file loads back as the
    tree the restatement builds from the frames' descriptors (device extractor, one document per frame)"""
    import subprocess
    import harness_seq
    from test_gpu_harness import _build
    from vo_slam_test_amd import synth
    n = 6
    grays, raws = harness_seq.render(n)
    seq = tmp_path / "seq"
    harness_seq.write(seq, grays, raws)
    exe = _build(tmp_path)
    cam = [str(float(c)) for c in synth.CAM] + [str(float(synth.DEPTH_SCALE))]
    out = tmp_path / "voc.dbow3"
    r = subprocess.run([str(exe), str(seq) + "/", str(tmp_path / "camera.txt"), "100", *cam, "--vocabulary-out", str(out)],
                       capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "vocabulary info: k = 10, L = 5" in r.stdout and "camera trajectory saved !!!" in r.stdout
    V, info = vo.load_vocabulary(out)
    ext = vo.OrbExtractor(1000, 1.2, 8, 20, 7)
    ds = [np.ascontiguousarray(ext(np.ascontiguousarray(g))[1]) for g in grays]
    ext.close()
    off = np.concatenate([[0], np.cumsum([len(d) for d in ds])]).astype(np.int32)
    ref = R.train(np.concatenate(ds), off, 10, 5, 0)
    tree = V.tree()
    V.close()
    assert info["k"] == 10 and info["L"] == 5 and info["n_nodes"] == ref["info"]["n_nodes"]
    for key in ("child_start", "children", "node_desc", "word_id", "node_weight"):
        assert np.array_equal(tree[key], ref[key]), key
