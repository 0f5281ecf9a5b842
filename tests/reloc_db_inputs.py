"""The relocalisation fixture (tests/reloc_inputs.py) as a key-frame store and database (test infrastructure): every
candidate of every frame becomes one key-frame, numbered frame-major; the ids of frame f's candidates are offset by
f * 2 * nk, so that they are globally unique and far outside [0, max_cand * nk)."""
import numpy as np

import kfdb_ref


def keyframes(fx):
    """-> (kfs: the store's key-frames in insertion order, lists: per frame the numbers of its candidates in walk order)"""
    kfs, lists = [], []
    for f, cl in enumerate(fx["candidates"]):
        lists.append(list(range(len(kfs), len(kfs) + len(cl))))
        for k in cl:
            g = dict(k)
            g["ids"] = (np.asarray(k["ids"], np.int64) + f * 2 * fx["nk"]).astype(np.int32)
            kfs.append(g)
    return kfs, lists


def dense_ids(cands):
    """the candidates of ONE frame with their global ids replaced by dense ones (what vo_tracker_set_reloc_candidates
    accepts) -> (candidates, table dense -> global)"""
    if not cands:
        return [], np.zeros(0, np.int32)
    table, inv = np.unique(np.concatenate([np.asarray(k["ids"], np.int32) for k in cands]), return_inverse=True)
    out, o = [], 0
    for k in cands:
        g = dict(k)
        g["ids"] = inv[o:o + len(k["ids"])].astype(np.int32)
        o += len(k["ids"])
        out.append(g)
    return out, table.astype(np.int32)


def bow(orc, vd, desc, levelsup=3):
    """(word, weight, node) per feature on the oracle"""
    n = len(desc)
    word, weight, node = np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32)
    if n:
        orc.lib().orc_bow_transform(int(vd["L"]), np.ascontiguousarray(vd["child_start"], np.int32), np.ascontiguousarray(vd["children"], np.int32),
                                    np.ascontiguousarray(vd["node_desc"], np.uint8), np.ascontiguousarray(vd["node_weight"], np.float64),
                                    np.ascontiguousarray(vd["word_id"], np.int32), n, np.ascontiguousarray(desc, np.uint8), levelsup, word,
                                    weight, node)
    return word, weight, node


def db_keyframes(orc, fx):
    """The store of the end-to-end test: keyframes() made visible to the database.  A KeyFrame holds EVERY feature of
    its image, with or without a map point, and its BoW vector comes from all of their descriptors; the fixture's
    candidates hold only the features that carry a map point, and give the ones the BoW search must not match a random
    descriptor -- so their vectors share too few words with any frame to pass the common-word gate of map.cpp:130-141.
    Here every key-frame covers its whole frame: a feature the BoW search must not match carries the centre of the
    vocabulary word its frame feature falls into (the same word for the database; ~ 128 bits from the frame's descriptor,
    far beyond TH 50, for the search), and the frame features a candidate does not hold are appended without a map
    point (flags 0: skipped by both searches).  -> (kfs, lists) as keyframes()"""
    vd = fx["vocab"]
    leaf_of_word = np.nonzero(np.asarray(vd["word_id"]) >= 0)[0]
    centres = np.asarray(vd["node_desc"], np.uint8)[leaf_of_word]  # [n_words][32]
    kfs, lists = keyframes(fx)
    out = []
    for f, ls in enumerate(lists):
        k_, d = fx["frames"][f][0], fx["frames"][f][1]
        word = bow(orc, vd, d)[0]
        n = len(d)
        for g in ls:
            k = kfs[g]
            idx = np.asarray(k["frame_index"])
            desc = np.asarray(k["desc"], np.uint8).copy()
            dist = np.unpackbits(desc ^ d[idx], axis=1).sum(1)
            far = dist > 50
            desc[far] = centres[word[idx[far]]]
            rest = np.setdiff1d(np.arange(n), idx)
            m = len(rest)
            cat = lambda a, b: np.concatenate([np.asarray(a), b])
            q = dict(k)
            q["frame_index"] = cat(idx, rest)
            q["desc"] = cat(desc, centres[word[rest]])
            q["angle"] = cat(k["angle"], k_["angle"][rest].astype(np.float32))
            q["flags"] = cat(k["flags"], np.zeros(m, np.uint8))
            q["points"] = cat(k["points"], np.zeros((m, 3)))
            q["ids"] = cat(k["ids"], np.zeros(m, np.int32))
            q["point_desc"] = cat(k["point_desc"], d[rest])
            q["min_dist"] = cat(k["min_dist"], np.zeros(m, np.float32))
            q["max_dist"] = cat(k["max_dist"], np.zeros(m, np.float32))
            q["nodes"] = bow(orc, vd, q["desc"])[2]
            out.append(q)
    return out, lists


def database(orc, fx, kfs, lists):
    """-> dict(n_words, vectors: per key-frame (words, values), neighbors: per key-frame list, queries: per frame (words,
    values)).  No covisibility lists: every group is one key-frame."""
    vd = fx["vocab"]
    vec = lambda desc: kfdb_ref.bow_vector(*bow(orc, vd, desc)[:2])
    vectors = [vec(k["desc"]) for k in kfs]
    neighbors = [[] for _ in kfs]  # (with the candidates of a frame as each other's neighbours every frame gets ONE candidate)
    queries = [vec(fr[1]) for fr in fx["frames"]]
    return dict(n_words=int((np.asarray(vd["word_id"]) >= 0).sum()), vectors=vectors, neighbors=neighbors, queries=queries)


def model_candidates(db):
    """kfdb_ref's Map::detectRelocalizationCandidates for every frame of the fixture -> per frame the key-frame numbers"""
    ref = kfdb_ref.Database()
    for w, v in db["vectors"]:
        ref.insert(w, v)
    for g, nb in enumerate(db["neighbors"]):
        ref.set_neighbors(g, nb)
    return [[int(c) for c in ref.query_reloc(w, v)[0]] for w, v in db["queries"]]
