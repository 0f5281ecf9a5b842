"""The numpy restatement of the vocabulary-training contract (tests/vocab_ref.py) against brute force, its
structural guarantees, the subtree property that carries batch invariance, and the drop-in boundary of the four new entry
points.  No GPU."""
import pathlib
import re

import numpy as np
import pytest

import vocab_inputs as I
import vocab_ref as R

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _as_int(d):
    return int.from_bytes(bytes(d), "little")


def _ham(a, b):
    return bin(_as_int(a) ^ _as_int(b)).count("1")


# ------------------------------------------------------------------------------------------------- against brute force
def test_assignment_is_the_true_arg_min_with_the_tie_rule():
    rng = np.random.default_rng(0)
    desc = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    centres = desc[rng.integers(0, 200, 9)].copy()
    centres[5] = centres[2]  # an exact tie between clusters 2 and 5: the lower index wins
    a = R.assign(desc, centres)
    for i, d in enumerate(desc):
        dist = [_ham(d, c) for c in centres]
        assert a[i] == dist.index(min(dist))
    assert 5 not in a


def test_majority_against_per_bit_counts():
    rng = np.random.default_rng(1)
    for m in (1, 2, 3, 4, 7, 10, 33):
        mem = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        got = _as_int(R.majority(mem))
        want = 0
        for b in range(256):
            cnt = sum((_as_int(d) >> b) & 1 for d in mem)
            if cnt >= m // 2 + m % 2:
                want |= 1 << b
        assert got == want
    two = np.zeros((2, 32), np.uint8)
    two[0, 0] = 1  # count 1 of 2 reaches 2 // 2 + 0: set (DBoW's rounding)
    assert _as_int(R.majority(two)) == 1


def test_kmeanspp_picks_against_an_explicit_prefix_walk():
    rng = np.random.default_rng(2)
    desc = rng.integers(0, 256, (150, 32), dtype=np.uint8)
    desc[40:60] = desc[7]  # duplicates: zero distance once 7 (or a copy) is a centre
    key = R.path_key(99, (3, 1))
    picks = R.seed_centres(desc, 6, key)
    want = [R.draw(key, 0) % len(desc)]
    for j in range(1, 6):
        md = [min(_ham(d, desc[c]) for c in want) for d in desc]
        total = sum(md)
        cut = 1 + R.draw(key, j) % total
        run = 0
        for i, x in enumerate(md):
            run += x
            if run >= cut:
                want.append(i)
                break
    assert list(picks) == want
    assert len({bytes(desc[i]) for i in picks}) == 6  # a descriptor at distance 0 of a centre is never drawn


def test_draw_is_keyed_by_seed_path_and_counter():
    assert R.mix(0) == 0xE220A8397B1DCDAF  # splitmix64's first output for state 0
    keys = {R.path_key(s, p) for s in (0, 1) for p in ((), (0,), (1,), (0, 0), (0, 1), (1, 0))}
    assert len(keys) == 12
    assert len({R.draw(R.path_key(5, (2,)), j) for j in range(32)}) == 32


# ----------------------------------------------------------------------------------------------------------- structure
def _structure(t, n, k, L):
    cs, ch, lvl = t["child_start"], t["children"], t["level"]
    nch = np.diff(cs)
    assert nch.max(initial=0) <= k and list(ch) == list(range(1, len(lvl)))
    leaves = np.nonzero(t["word_id"] >= 0)[0]
    assert np.array_equal(t["word_id"][leaves], np.arange(len(leaves))) and (nch[leaves] == 0).all()
    assert (nch[t["word_id"] < 0][1:] > 0).all()  # an inner node has children
    assert n == 0 or (t["word_id"][t["leaf_of"]] >= 0).all()  # every descriptor reaches exactly one leaf
    held = np.bincount(t["leaf_of"], minlength=len(lvl)) if n else np.zeros(len(lvl), int)
    assert ((held[leaves] <= 1) | (lvl[leaves] == L)).all()  # no leaf above level L holds more than one descriptor
    assert lvl.max() <= L and t["info"]["n_capped"] == 0


@pytest.mark.parametrize("k,L", I.KL)
def test_structure_and_partition(k, L):
    for n in (0, 1, k, k + 1, 65, 1500):
        desc = I.uniform(n, seed=n)
        t = R.train(desc, I.offsets(n, 5), k, L, seed=1)
        _structure(t, n, k, L)
        if 0 < n <= k:
            assert t["info"]["n_nodes"] == n + 1 and np.array_equal(t["node_desc"][1:], desc)  # one child per descriptor
        # descending the tree with the BoW tests' numpy transform reproduces the training partition
        assert np.array_equal(R.transform(t, desc), t["leaf_of"])


def test_duplicates_only_input_ends_with_fewer_children():
    desc = I.all_equal(500)
    t = R.train(desc, I.offsets(500, 3), 10, 5, seed=0)
    # one centre at every level (sum == 0 at the first draw); the single child holds everything and is clustered again
    # down to level L: a chain of L nodes below the root, one word
    assert t["info"]["n_nodes"] == 6 and t["info"]["n_words"] == 1 and (t["node_desc"][1:] == desc[0]).all()
    assert np.diff(t["child_start"]).tolist() == [1, 1, 1, 1, 1, 0]
    few = I.duplicates(3000, distinct=4)
    t = R.train(few, I.offsets(3000, 3), 10, 5, seed=0)
    assert np.diff(t["child_start"])[0] == 4  # sum == 0 after four centres
    _structure(t, 3000, 10, 5)
    assert t["info"]["n_words"] == 4 and (t["node_weight"] == 0).all()  # every word is seen in every image: log(3 / 3)


def test_subtree_is_a_function_of_seed_path_and_ordered_members():
    n, k, L, seed = 4000, 6, 4, 21
    desc = I.clustered(n, seed=1)
    t = R.train(desc, I.offsets(n, 10), k, L, seed)
    cs, ch = t["child_start"], t["children"]
    # the members of level-1 cluster c, in input order: the descriptors whose leaf lies below child c of the root
    top = np.zeros(len(t["level"]), np.int64)
    parent = np.zeros(len(top), np.int64)
    for p in range(len(top)):
        parent[ch[cs[p]:cs[p + 1]]] = p
    for node in range(1, len(top)):
        top[node] = node if parent[node] == 0 else top[parent[node]]
    for c in (0, 3, k - 1):
        child = ch[cs[0] + c]
        members = np.nonzero(top[t["leaf_of"]] == child)[0]
        sub = R.subtree(desc, members, k, L, seed, (c,), 1)
        below = np.nonzero(top == child)[0]  # ascending node ids = breadth-first within the subtree
        assert len(below) == len(sub["level"])
        assert np.array_equal(sub["node_desc"][1:], t["node_desc"][below[1:]])
        assert np.array_equal(np.diff(sub["child_start"]), np.diff(cs)[below])
        assert np.array_equal(below[sub["leaf_of"][members]], t["leaf_of"][members])
    # ... whatever else is trained beside it: the same members inside another training set
    other = np.concatenate([desc[members], I.uniform(50, seed=5)])
    assert not np.array_equal(R.train(other, I.offsets(len(other), 2), k, L, seed)["node_desc"][:5], t["node_desc"][:5])


def test_weights_are_the_idf_of_the_training_transform():
    import math
    n, k, L = 1200, 5, 3
    desc, off = I.clustered(n, seed=3), I.offsets(n, 6)
    t = R.train(desc, off, k, L, seed=4)
    image = np.searchsorted(off, np.arange(n), side="right") - 1
    for w in np.nonzero(t["word_id"] >= 0)[0][:40]:
        imgs = {int(image[i]) for i in np.nonzero(t["leaf_of"] == w)[0]}
        assert t["node_weight"][w] == (math.log(6 / len(imgs)) if imgs else 0.0)
    assert (t["node_weight"][t["word_id"] < 0] == 0).all()


# ------------------------------------------------------------------------------------------------- the cap and the golden
def test_iteration_cap_has_its_margin_on_the_fixtures(orc):
    """VO_VOCAB_MAX_LLOYD >= 8 x the worst iteration count over the inputs of tests/test_gpu_vocab_train.py, same seeds (the
    200 000 case, which takes this restatement half a minute, is run by the GPU test: 25 iterations there, n_capped == 0)"""
    worst = 0
    p = orc.orb_params()
    ext, ext_off = I.extracted(lambda img: orc.extract(p, img)[:2], 6)
    for k, L in I.KL:
        sets = [(I.uniform(20000, seed=20000 + k), I.offsets(20000, 7), 3), (I.uniform(1000, seed=1000 + k), I.offsets(1000, 7), 3),
                (I.clustered(6000, seed=k), I.offsets(6000, 40), 9), (I.duplicates(6000, seed=k), I.offsets(6000, 40), 9),
                (I.all_equal(6000, seed=k), I.offsets(6000, 40), 9), (ext, ext_off, 5)]
        for desc, off, seed in sets:
            info = R.train(desc, off, k, L, seed=seed)["info"]
            assert info["n_capped"] == 0
            worst = max(worst, info["lloyd_iterations_max"])
    print("worst Lloyd iteration count", worst)
    assert R.MAX_LLOYD >= 8 * max(worst, 25)
    header = (ROOT / "include" / "vo_hip.h").read_text()
    assert int(re.search(r"#define VO_VOCAB_MAX_LLOYD (\d+)", header).group(1)) == R.MAX_LLOYD


def test_golden_tree_pins_the_restatement():
    g = np.load(ROOT / "tests" / "golden" / "g12_vocab_train.npz")
    t = R.train(g["desc"], g["image_offsets"], int(g["k"]), int(g["L"]), int(g["seed"]))
    for key in ("child_start", "children", "node_desc", "word_id", "node_weight"):
        assert np.array_equal(t[key], g[key]), key
    assert [t["info"][x] for x in ("n_nodes", "n_words", "n_levels", "lloyd_iterations_max", "n_capped")] == g["info"].tolist()


# --------------------------------------------------------------------------------------------------- drop-in boundary
def test_new_entry_points_are_declared_and_bound(vo):
    header = (ROOT / "include" / "vo_hip.h").read_text()
    for name in ("vo_vocab_train", "vo_vocab_train_dev", "vo_vocab_tree", "vo_vocab_save"):
        assert name in vo.SYMBOLS and re.search(r"\b%s\s*\(" % name, header) and hasattr(vo.lib(), name)
    assert "map.cpp:60-99" in header
    assert callable(vo.train_vocabulary) and hasattr(vo.Vocabulary, "tree") and hasattr(vo.Vocabulary, "save")
