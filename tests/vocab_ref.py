"""numpy restatement of the vocabulary-training contract of DESIGN.md §4d: DBoW3::Vocabulary::create (k-majority tree:
HKmeansStep, initiateClustersKMpp, DescManip::meanValue, createWords, setNodeWeights) as Map::createVocabulary calls it
(reference map.cpp:60-99), written from DBoW2/DBoW3's published algorithm with the deviations §4d states (integer
k-means++ draw keyed by the node's path, breadth-first node ids, an iteration cap).  Everything but the final log is integer
arithmetic: vo_vocab_train must reproduce child_start / children / node_desc / word_id / info exactly."""
from __future__ import annotations

import math

import numpy as np

MASK64 = (1 << 64) - 1
MAX_LLOYD = 2048  # VO_VOCAB_MAX_LLOYD (include/vo_hip.h)


# ----------------------------------------------------------------------------------------------------------------- draw
def mix(z: int) -> int:
    """splitmix64's step: add the golden-ratio increment, then its finaliser"""
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def path_key(seed: int, path=()) -> int:
    """key of the node reached from the root by the child indices `path`"""
    h = mix(seed & MASK64)
    for c in path:
        h = mix(h ^ (int(c) + 1))
    return h


def draw(key: int, j: int) -> int:
    return mix((mix(key) + j) & MASK64)


# ------------------------------------------------------------------------------------------------------------- distances
def hamming(desc: np.ndarray, centre: np.ndarray) -> np.ndarray:
    """[m] Hamming distances of desc [m, 32] to one 32-byte centre"""
    a = np.ascontiguousarray(desc, np.uint8).view(np.uint64).reshape(len(desc), 4)
    b = np.ascontiguousarray(centre, np.uint8).view(np.uint64).reshape(1, 4)
    return np.bitwise_count(a ^ b).sum(axis=1).astype(np.int64)


def assign(desc: np.ndarray, centres: np.ndarray) -> np.ndarray:
    """nearest centre per descriptor, ties to the lowest cluster index (np.argmin returns the first minimum)"""
    d = np.stack([hamming(desc, c) for c in centres], axis=1)
    return np.argmin(d, axis=1).astype(np.int32)


def majority(members: np.ndarray) -> np.ndarray:
    """DescManip::meanValue: bit set iff its count >= m / 2 + m % 2"""
    m = len(members)
    cnt = np.unpackbits(np.ascontiguousarray(members, np.uint8), axis=1, bitorder="little").sum(axis=0, dtype=np.int64)
    return np.packbits((cnt >= m // 2 + m % 2).astype(np.uint8), bitorder="little")


def seed_centres(desc: np.ndarray, k: int, key: int) -> np.ndarray:
    """initiateClustersKMpp with the integer draw: indices (into desc) of the <= k initial centres"""
    m = len(desc)
    picks = [draw(key, 0) % m]
    min_dist = hamming(desc, desc[picks[0]])
    for j in range(1, k):
        total = int(min_dist.sum())
        if total == 0:
            break
        cut = 1 + draw(key, j) % total
        i = int(np.searchsorted(np.cumsum(min_dist), cut, side="left"))  # first i whose running sum reaches cut
        picks.append(i)
        min_dist = np.minimum(min_dist, hamming(desc, desc[i]))
    return np.array(picks, np.int64)


def cluster(desc: np.ndarray, k: int, key: int, max_lloyd: int = MAX_LLOYD):
    """one clustering step: (centres [c, 32], assignment [m], iterations, capped)"""
    m = len(desc)
    if m <= k:
        return desc.copy(), np.arange(m, dtype=np.int32), 0, False
    centres = desc[seed_centres(desc, k, key)].copy()
    prev, it = None, 0
    while True:
        a = assign(desc, centres)
        it += 1
        if prev is not None and np.array_equal(a, prev):
            return centres, a, it, False
        if it == max_lloyd:
            return centres, a, it, True
        prev = a
        for c in range(len(centres)):
            mem = desc[a == c]
            if len(mem):
                centres[c] = majority(mem)  # an empty cluster keeps its centre


# ------------------------------------------------------------------------------------------------------------------ tree
def _grow(desc, idx, k, L, seed, path0, level0, max_lloyd):
    """breadth-first growth below one node holding the descriptors `idx` (input order).  Returns flat arrays with the start
    node as node 0, the leaf of every descriptor of idx, and (iterations max, capped count, deepest level)."""
    node_desc = [np.zeros(32, np.uint8)]
    level, kids = [level0], [[]]
    leaf_of = np.zeros(len(desc), np.int64)
    frontier = [(0, np.asarray(idx, np.int64), tuple(path0))]
    it_max = capped = 0
    while frontier:
        nxt = []
        for node, members, path in frontier:  # node-id order
            centres, a, it, cap = cluster(desc[members], k, path_key(seed, path), max_lloyd)
            it_max, capped = max(it_max, it), capped + int(cap)
            for c in range(len(centres)):
                child = len(node_desc)
                node_desc.append(centres[c])
                level.append(level[node] + 1)
                kids.append([])
                kids[node].append(child)
                mem = members[a == c]
                leaf_of[mem] = child
                if level[child] < L and len(mem) > 1:
                    nxt.append((child, mem, path + (c,)))
        frontier = nxt
    n = len(node_desc)
    cs = np.zeros(n + 1, np.int32)
    cs[1:] = np.cumsum([len(x) for x in kids])
    children = np.array([c for x in kids for c in x], np.int32)
    word_id = np.full(n, -1, np.int32)
    leaves = [i for i in range(1, n) if not kids[i]]
    word_id[leaves] = np.arange(len(leaves), dtype=np.int32)
    return dict(child_start=cs, children=children, node_desc=np.ascontiguousarray(np.array(node_desc, np.uint8).reshape(n, 32)),
                word_id=word_id, level=np.array(level, np.int32), leaf_of=leaf_of, it_max=it_max, capped=capped)


def subtree(desc, idx, k, L, seed, path, level, max_lloyd=MAX_LLOYD):
    """the subtree below the node at `path` (depth `level`) that holds the descriptors idx, node 0 = that node"""
    return _grow(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), idx, k, L, seed, path, level, max_lloyd)


def transform(tree, desc) -> np.ndarray:
    """DBoW3::Vocabulary::transform's descent: the leaf node of every descriptor (strict <: the first minimum wins)"""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    cs, ch, nd = tree["child_start"], tree["children"], tree["node_desc"]
    node = np.zeros(len(desc), np.int64)
    active = np.arange(len(desc))
    while len(active):
        still = []
        for p in np.unique(node[active]):
            kids = ch[cs[p]:cs[p + 1]]
            if len(kids) == 0:
                continue
            sel = active[node[active] == p]
            node[sel] = kids[assign(desc[sel], nd[kids])]
            still.append(sel)
        active = np.concatenate(still) if still else np.zeros(0, np.int64)
    return node


def train(desc, image_offsets, k=10, L=5, seed=0, max_lloyd=MAX_LLOYD):
    """the whole contract: dict(child_start, children, node_desc, node_weight, word_id, L, k, level, leaf_of, info)"""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    off = np.asarray(image_offsets, np.int64)
    n, n_images = len(desc), len(off) - 1
    assert k >= 2 and L >= 1 and off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
    if n == 0:
        t = dict(child_start=np.zeros(2, np.int32), children=np.zeros(0, np.int32), node_desc=np.zeros((1, 32), np.uint8),
                 word_id=np.full(1, -1, np.int32), level=np.zeros(1, np.int32), leaf_of=np.zeros(0, np.int64), it_max=0, capped=0)
    else:
        t = _grow(desc, np.arange(n), k, L, seed, (), 0, max_lloyd)
    # setNodeWeights: idf over the images, by transform of the training set (not by the partition)
    weight = np.zeros(len(t["word_id"]))
    if n:
        words = transform(t, desc)
        image = np.searchsorted(off, np.arange(n), side="right") - 1
        pairs = np.unique(np.stack([words, image], axis=1), axis=0)
        ni = np.bincount(pairs[:, 0], minlength=len(weight))
        for w in np.nonzero((ni > 0) & (t["word_id"] >= 0))[0]:
            weight[w] = math.log(n_images / int(ni[w]))
    t.update(node_weight=weight, k=k, L=L,
             info=dict(n_nodes=len(t["word_id"]), n_words=int((t["word_id"] >= 0).sum()), n_levels=int(t["level"].max()),
                       lloyd_iterations_max=int(t["it_max"]), n_capped=int(t["capped"])))
    return t
